// C++ drop-in test of include/MeshFEMHip/MassProperties.hh and the per-element overload of Eigensolver.hh on a quadratic tet Simulator clamped on
// its face x = min, bimaterial: density 1 where the element centroid has x < the middle of the box, 8 elsewhere. Writes the eigenvalues and the
// mass properties; tests/test_cpp_density.py compares them with the Python layer's on the same mesh.
// argv: device ordinal, mesh file (i64 nVert, i64 nElem, f64 V[nVert][3], i32 T[nElem][4]), nev, output file (f64 lambda[nev], mass, com[3],
// S[3][3], inertia[3][3], then (M x)[nDoF][3] for x = the node positions).
#include <MeshFEMHip/Eigensolver.hh>
#include <MeshFEMHip/MassProperties.hh>
#include <algorithm>
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
        using Sim = LinearElasticity::Simulator<3, 2>;
        Sim sim(T, V, device);
        sim.setIsotropicMaterial(1.0, 0.3);
        check(sim.ctx(), mfh_set_option(sim.ctx(), "deterministic", 1.0));       // bit-reproducible: the test compares with another process
        sim.applyDirichletBox({-1e-9, -1e-9, -1e-9}, {1e-9, 1.0 + 1e-9, 1.0 + 1e-9}, {0, 0, 0}, true);
        Real lo = V[0][0], hi = V[0][0];
        for (const auto &p : V) { lo = std::min(lo, p[0]); hi = std::max(hi, p[0]); }
        std::vector<Real> rho(T.size());
        for (size_t e = 0; e < T.size(); ++e) {
            Real x = 0;
            for (int k = 0; k < 4; ++k) x += V[(size_t)T[e][k]][0];
            rho[e] = 0.25 * x < 0.5 * (lo + hi) ? 1.0 : 8.0;
        }
        mfh_modes_info info{};
        const auto r = vibrationalModes(sim, nev, rho, false, ModesOptions(), &info);
        if (r.first.size() != (size_t)nev || r.second.size() != (size_t)nev || r.second[0].size() != sim.numDoFs() || !info.converged) {
            printf("FAILED: sizes / convergence\n");
            return 2;
        }
        const auto p = massProperties(sim);                                        // the field of the overload stays in force
        setDensity(sim, std::vector<Real>());
        const auto unit = massProperties(sim);
        if (!(unit.mass < p.mass && p.mass < 8.0 * unit.mass)) { printf("FAILED: the mass %g against %g at unit density\n", p.mass, unit.mass); return 2; }
        setDensity(sim, rho);
        Sim::VField x(sim.numDoFs());
        int64_t nElem, nNode;
        check(sim.ctx(), mfh_mesh_sizes(sim.ctx(), &nElem, &nNode, nullptr, nullptr, nullptr, nullptr, nullptr));
        std::vector<Real> pos((size_t)nNode * 3);
        check(sim.ctx(), mfh_mesh_get_node_positions(sim.ctx(), pos.data()));
        for (size_t i = 0; i < x.size(); ++i) x[i] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
        const auto Mx = applyMass(sim, x);
        if (argc > 4) {
            FILE *f = fopen(argv[4], "wb");
            if (!f) { printf("cannot write %s\n", argv[4]); return 2; }
            fwrite(r.first.data(), sizeof(Real), r.first.size(), f);
            fwrite(&p.mass, sizeof(Real), 1, f);
            fwrite(p.com.data(), sizeof(Real), 3, f);
            fwrite(&p.secondMoment[0][0], sizeof(Real), 9, f);
            fwrite(&p.inertia[0][0], sizeof(Real), 9, f);
            fwrite(&Mx[0][0], sizeof(Real), 3 * Mx.size(), f);
            fclose(f);
        }
        printf("lambda[0] %.17g, mass %.17g\n", r.first[0], p.mass);
        printf("density ok\n");
    } catch (const std::runtime_error &e) {
        printf("runtime_error: %s\n", e.what());
        return 3;
    }
    return 0;
}
