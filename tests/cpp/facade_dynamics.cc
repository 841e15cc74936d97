// C++ drop-in test of include/MeshFEMHip/Dynamics.hh on a quadratic tet Simulator clamped on its face x = min and pulled on its face x = max: writes
// what two chained calls of transient (the second started from the first's u, v, a) return; tests/test_cpp_dynamics.py compares it with the Python layer's on the same mesh.
// argv: device ordinal, mesh file (i64 nVert, i64 nElem, f64 V[nVert][3], i32 T[nElem][4]), nSteps, dt, density, output file (f64 u[nDoF][3],
// v[nDoF][3], a[nDoF][3], probes[nSteps + 1][2], energies[nSteps + 1][3], then the snapshots of every second step).
#include <MeshFEMHip/Dynamics.hh>
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
    const int nSteps = argc > 3 ? atoi(argv[3]) : 2;
    const Real dt = argc > 4 ? atof(argv[4]) : 0.1;
    const Real density = argc > 5 ? atof(argv[5]) : 1.0;
    try {
        using Sim = LinearElasticity::Simulator<3, 2>;
        Sim sim(T, V, device);
        sim.setIsotropicMaterial(1.0, 0.3);
        check(sim.ctx(), mfh_set_option(sim.ctx(), "deterministic", 1.0));       // bit-reproducible: the test compares with another process
        sim.applyDirichletBox({-1e-9, -1e-9, -1e-9}, {1e-9, 1.0 + 1e-9, 1.0 + 1e-9}, {0, 0, 0}, true);
        sim.applyNeumannBox({1.0 - 1e-9, -1e-9, -1e-9}, {1.0 + 1e-9, 1.0 + 1e-9, 1.0 + 1e-9}, {0.0, 0.0, -1.0}, MFH_NEUMANN_TRACTION, true);
        TransientOptions<Sim::VField> opt;
        opt.density = density;
        opt.rayleighMass = 0.05; opt.rayleighStiff = 0.01;
        opt.rtol = 1e-10;
        for (int k = 0; k <= nSteps; ++k) opt.amplitude.push_back(k % 3 == 0 ? 1.0 : 0.5);
        opt.probes = {{sim.numDoFs() - 1, 2}, {sim.numDoFs() / 2, 0}};
        opt.snapshotStride = 2;
        opt.energies = true;
        // two chained halves through (u0, v0, a0): the second continues the first, and together they are the run of nSteps steps
        const int half = nSteps / 2;
        const std::vector<Real> amp = opt.amplitude;
        opt.amplitude.assign(amp.begin(), amp.begin() + half + 1);
        const auto r1 = transient(sim, dt, half, opt);
        opt.amplitude.assign(amp.begin() + half, amp.end());
        opt.u0 = r1.u; opt.v0 = r1.v; opt.a0 = r1.a;
        auto r = transient(sim, dt, nSteps - half, opt);
        if (r1.info.stepsDone != half || r.info.stepsDone != nSteps - half || r.info.iterationsInit != 0 || half % 2 != 0 || r.probes.empty() || r.snapshots.empty()) {
            printf("FAILED: steps of the halves\n");
            return 2;
        }
        r.probes.insert(r.probes.begin(), r1.probes.begin(), r1.probes.end() - 1);
        r.energies.insert(r.energies.begin(), r1.energies.begin(), r1.energies.end() - 1);
        r.snapshots.insert(r.snapshots.begin(), r1.snapshots.begin(), r1.snapshots.end() - 1);
        if (r.u.size() != sim.numDoFs() || r.probes.size() != (size_t)nSteps + 1 || r.snapshots.size() != (size_t)nSteps / 2 + 1 ||
            r.energies.size() != (size_t)nSteps + 1) {
            printf("FAILED: sizes / steps\n");
            return 2;
        }
        if (argc > 6) {
            FILE *f = fopen(argv[6], "wb");
            if (!f) { printf("cannot write %s\n", argv[6]); return 2; }
            for (const auto *x : {&r.u, &r.v, &r.a}) fwrite(&(*x)[0][0], sizeof(Real), 3 * x->size(), f);
            for (const auto &p : r.probes) fwrite(p.data(), sizeof(Real), p.size(), f);
            for (const auto &e : r.energies) fwrite(e.data(), sizeof(Real), 3, f);
            for (const auto &s : r.snapshots) fwrite(&s[0][0], sizeof(Real), 3 * s.size(), f);
            fclose(f);
        }
        printf("%d + %d steps, %d PCG iterations in the second half (worst step %d), note: %s\n", half, (int)r.info.stepsDone, (int)r.info.iterationsTotal, (int)r.info.iterationsMax, r.info.note);
        printf("transient ok\n");
    } catch (const std::runtime_error &e) {
        printf("runtime_error: %s\n", e.what());
        return 3;
    }
    return 0;
}
