// C++ drop-in test of include/MeshFEMHip/VolumeLoads.hh and Simulator::perElementStressFieldLoad on a quadratic tet mesh of the box [0,1] x [0,1] x [0,L]:
// the hanging column (nu = 0, clamped at z = 0, body force rho g e_z: u_z = rho g / E (L z - z^2 / 2)), the free thermal expansion of the same box
// (u = alpha dT (x - mean of the nodes), no stress), and two load vectors written out for tests/test_cpp_volume_loads.py to compare with the Python layer's.
// argv: device ordinal, mesh file (i64 nVert, i64 nElem, f64 V[nVert][3], i32 T[nElem][4]), L, output file (f64 body[nDoF][3], stress[nDoF][3]).
#include <MeshFEMHip/VolumeLoads.hh>
#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace MeshFEMHip;
using Sim = LinearElasticity::Simulator<3, 2>;

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
    const Real L = argc > 3 ? atof(argv[3]) : 1.0;
    try {
        const Real E = 50.0, rho = 2.5, g = 9.81, alpha = 2.0e-3, dT = 35.0;
        {   // hanging column
            Sim sim(T, V, device);
            sim.setIsotropicMaterial(E, 0.0);
            sim.applyDirichletBox({-1e-9, -1e-9, -1e-9}, {1.0 + 1e-9, 1.0 + 1e-9, 1e-9}, {0, 0, 0}, false);
            sim.rtol = 1e-12;
            const auto u = sim.solve(gravityLoad(sim, {0.0, 0.0, g}, rho));
            const auto x = sim.nodes();
            Real err = 0, scale = 0;
            for (size_t n = 0; n < u.size(); ++n) {
                const Real ref[3] = {0.0, 0.0, rho * g / E * (L * x[n][2] - 0.5 * x[n][2] * x[n][2])};
                for (int a = 0; a < 3; ++a) { err = std::max(err, std::fabs(u[n][a] - ref[a])); scale = std::max(scale, std::fabs(ref[a])); }
            }
            printf("hanging column: error %.2e of max|u| %.3e\n", err / scale, scale);
            if (!(err <= 1e-9 * scale)) { printf("FAILED: hanging column\n"); return 2; }
            printf("column ok\n");
        }
        Sim sim(T, V, device);
        sim.setIsotropicMaterial(E, 0.3);
        {   // free thermal expansion
            sim.applyNoRigidMotionConstraint();
            sim.rtol = 1e-12;
            const std::vector<Real> al(sim.numElements(), alpha), dt(sim.numElements(), dT);
            const auto u = sim.solve(thermalLoad(sim, al, dt));
            const auto x = sim.nodes();
            std::array<Real, 3> mean = {0, 0, 0};
            for (const auto &p : x)
                for (int a = 0; a < 3; ++a) mean[a] += p[a] / (Real)x.size();
            Real err = 0, scale = 0;
            for (size_t n = 0; n < u.size(); ++n)
                for (int a = 0; a < 3; ++a) {
                    const Real ref = alpha * dT * (x[n][a] - mean[a]);
                    err = std::max(err, std::fabs(u[n][a] - ref)); scale = std::max(scale, std::fabs(ref));
                }
            Real smax = 0;
            for (Real s : thermalStress(sim, u, al, dt)) smax = std::max(smax, std::fabs(s));
            printf("free expansion: error %.2e of max|u|, thermal stress %.2e of E alpha dT\n", err / scale, smax / (E * alpha * dT));
            if (!(err <= 1e-9 * scale) || !(smax <= 1e-9 * E * alpha * dT)) { printf("FAILED: free expansion\n"); return 2; }
            printf("expansion ok\n");
        }
        // two loads of fields that the Python side rebuilds from the node positions and the element indices
        const auto x = sim.nodes();
        Sim::VField b(x.size());
        for (size_t n = 0; n < x.size(); ++n) b[n] = {x[n][0] * x[n][1], x[n][2], x[n][0] + 2.0 * x[n][1]};
        std::vector<Real> density(sim.numElements());
        Sim::SMField sigma(sim.numElements());
        for (size_t e = 0; e < sigma.size(); ++e) {
            density[e] = 1.0 + 0.25 * (Real)(e % 3);
            for (size_t k = 0; k < 6; ++k) sigma[e][k] = (Real)((7 * e + 3 * k) % 11) / 11.0 - 0.5;
        }
        const auto body = bodyForceLoad(sim, b, density);
        const auto stress = sim.perElementStressFieldLoad(sigma);
        if (body.size() != sim.numDoFs() || stress.size() != sim.numDoFs()) { printf("FAILED: sizes\n"); return 2; }
        if (argc > 4) {
            FILE *f = fopen(argv[4], "wb");
            if (!f) { printf("cannot write %s\n", argv[4]); return 2; }
            fwrite(&body[0][0], sizeof(Real), 3 * body.size(), f);
            fwrite(&stress[0][0], sizeof(Real), 3 * stress.size(), f);
            fclose(f);
        }
        printf("volume loads ok\n");
    } catch (const std::runtime_error &e) {
        printf("runtime_error: %s\n", e.what());
        return 3;
    }
    return 0;
}
